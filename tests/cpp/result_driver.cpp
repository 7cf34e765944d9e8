// Stand-alone sanitizer program for the result builder (fg_program_result, fg_program::compile_results in fg_program.cpp): built from
// the host sources with -fsanitize=address,undefined and run as a child process by tests/test_result_cpu.py.  It feeds the builder
// well-formed result expressions -- every token kind, linear predictors long enough to fuse -- and corrupted token streams
// (truncated, stack underflow, FG_T_SELECT with a bad option count, site handle out of range, unknown token), checks every return
// code, and walks the compiled instruction list the way k_result_eval does: every slot an instruction touches must lie inside the
// result slot file, every fused term inside the result pool, one FG_OP_FACTOR per result.
//   result_driver <seed>   ->   "results ok <accepted> refused <refused> programs <n>", exit 0; exit 1 with a message on a violation
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "../../include/fugue_amd.h"
#include "../../fugue_amd/csrc/fg_program.h"

static fg_tok tok(int op, int a = 0, double imm = 0.0) { fg_tok t; std::memset(&t, 0, sizeof t); t.op = op; t.a = a; t.imm = imm; return t; }

static int fail(const char *what, int got) { std::printf("VIOLATION %s (got %d: %s)\n", what, got, fg_last_error()); std::fflush(stdout); return 1; }

// the compiled list, as the kernel reads it
static const char *walk(const fg_program *p) {
    const int ns = p->res_n_slots;
    int factors = 0;
    if ((int)p->res_ins.size() != p->res_n_ins + 2) return "no two readable instructions past the list";
    auto slot_ok = [&](uint32_t w) { const uint32_t k = FG_OPND_KIND(w); return k == FG_OPND_IMM || ((k == FG_OPND_SLOT_F || k == FG_OPND_SLOT_I) && (int)FG_OPND_IDX(w) < ns - 1); };
    for (int pc = 0; pc < p->res_n_ins; ++pc) {
        const FgIns &I = p->res_ins[pc];
        const uint32_t code = FG_INS_OPCODE(I.op);
        if (code < FG_OP_FACTOR || code > FG_OP_DOT || code == FG_OP_CONSTLIK) return "an opcode the result kernel does not evaluate";
        if (code == FG_OP_FACTOR) ++factors;
        if (code == FG_OP_STORE) { if ((int)I.aux < (int)p->res_sites.size() || (int)I.aux >= ns - 1) return "STORE outside the temporaries"; continue; }
        if (code == FG_OP_GATHER) { if ((int)I.opnd[1] < 1 || (int)I.aux < (int)p->res_sites.size() || (int)(I.aux + I.opnd[1]) > ns - 1) return "GATHER options outside the temporaries"; continue; }
        if (code == FG_OP_DOT) {
            if ((size_t)I.aux + 2 * (size_t)I.opnd[1] > p->res_pool.size() || (I.aux & 1)) return "DOT terms outside the pool";
            for (uint32_t t = 0; t < I.opnd[1]; ++t) { const long long s = fg_as_i64(p->res_pool[I.aux + 2 * t]); if (s < 0 || s >= (long long)p->res_sites.size()) return "DOT term reads no site slot"; }
            continue;
        }
        if (!slot_ok(I.opnd[0])) return "operand 0 outside the slot file";
        if ((code == FG_OP_CLAMP || code == FG_OP_MAC) && !slot_ok(I.opnd[1])) return "operand 1 outside the slot file";
    }
    if (factors != (int)p->results.size()) return "not one FG_OP_FACTOR per result";
    for (size_t k = 0; k + 1 < p->res_sites.size(); ++k) if (p->res_sites[k] >= p->res_sites[k + 1]) return "result sites not ascending";
    return nullptr;
}

int main(int argc, char **argv) {
    std::mt19937_64 g(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    int accepted = 0, refused = 0, programs = 0;
    for (int rep = 0; rep < 200; ++rep) {
        fg_program *p = fg_program_new();
        const double dat[3] = {0.5, -1.25, 3.0};
        fg_program_data(p, "y", dat, 3);
        const int S = 1 + (int)(g() % 12);
        const fg_tok npar[2] = { tok(FG_T_CONST, 0, 0.0), tok(FG_T_CONST, 0, 1.0) };
        const int32_t plen2[2] = {1, 1};
        const fg_tok cpar[3] = { tok(FG_T_CONST, 0, 0.25), tok(FG_T_CONST, 0, 0.25), tok(FG_T_CONST, 0, 0.5) };
        const int32_t plen3[3] = {1, 1, 1};
        const fg_tok bpar[1] = { tok(FG_T_CONST, 0, 0.5) };
        const int32_t plen1[1] = {1};
        for (int j = 0; j < S; ++j) {
            char addr[16]; std::snprintf(addr, sizeof addr, "s#%d", (S - j) * 7 % 13 * 100 + j);    // address order != program order
            const int kind = (int)(g() % 4);
            const int h = kind == 0 ? fg_program_sample(p, addr, FG_CATEGORICAL, cpar, plen3, 3) : kind == 1 ? fg_program_sample(p, addr, FG_BERNOULLI, bpar, plen1, 1)
                                                                                                            : fg_program_sample(p, addr, FG_NORMAL, npar, plen2, 2);
            if (h != j) return fail("sample handle", h);
        }
        // a well-formed expression over every token kind
        std::function<void(std::vector<fg_tok> &, int)> expr = [&](std::vector<fg_tok> &t, int depth) {
            const int kind = depth <= 0 ? (int)(g() % 3) : (int)(g() % 8);
            if (kind == 0) t.push_back(tok(FG_T_CONST, 0, (double)((long long)(g() % 400) - 200) / 64.0));
            else if (kind == 1) t.push_back(tok(FG_T_SITE, (int)(g() % S)));
            else if (kind == 2) { fg_tok q = tok(FG_T_DATA, 0); q.b = (int)(g() % 3); t.push_back(q); }
            else if (kind == 3) { expr(t, depth - 1); t.push_back(tok(FG_T_NEG + (int)(g() % 9))); }
            else if (kind == 4) { expr(t, depth - 1); expr(t, depth - 1); t.push_back(tok(FG_T_ADD + (int)(g() % 7))); }
            else if (kind == 5) { expr(t, depth - 1); expr(t, depth - 1); expr(t, depth - 1); t.push_back(tok(FG_T_CLAMP)); }
            else if (kind == 6) { const int k = 1 + (int)(g() % 4); expr(t, depth - 1); for (int q = 0; q < k; ++q) expr(t, depth - 1); t.push_back(tok(FG_T_SELECT, k)); }
            else {                                         // a linear predictor: a run of `+ site * constant`, long enough to fuse into FG_OP_DOT (with a tail)
                const int terms = 1 + (int)(g() % 11);
                t.push_back(tok(FG_T_CONST, 0, 0.5));
                for (int q = 0; q < terms; ++q) { t.push_back(tok(FG_T_SITE, (int)(g() % S))); t.push_back(tok(FG_T_CONST, 0, 0.125 * (q + 1))); t.push_back(tok(FG_T_MUL)); t.push_back(tok(FG_T_ADD)); }
            }
        };
        int R = 0;
        const int want_results = (int)(g() % 5);
        for (int r = 0; r < want_results; ++r) {
            std::vector<fg_tok> t;
            expr(t, 3);
            std::string name = "result[" + std::to_string(R) + "]";
            const int corrupt = (int)(g() % 8);           // 0 .. 4: one corruption; else intact
            int expect_bad = 0;
            if (corrupt == 0) { if (!(t.back().op >= FG_T_NEG && t.back().op <= FG_T_TANH)) { t.pop_back(); expect_bad = 1; } }   // truncated: nothing, or operands left on the stack (a unary's operand alone is well formed)
            else if (corrupt == 1) { t.insert(t.begin(), tok(FG_T_ADD)); expect_bad = 1; }                        // stack underflow
            else if (corrupt == 2) { t.push_back(tok(FG_T_SELECT, (g() % 2) ? 0 : (int)t.size() + 5)); expect_bad = 1; }   // bad option count
            else if (corrupt == 3) { t.push_back(tok(FG_T_SITE, (g() % 2) ? S + (int)(g() % 9) : -1 - (int)(g() % 9))); t.push_back(tok(FG_T_ADD)); expect_bad = 1; }   // handle out of range
            else if (corrupt == 4) { t.push_back(tok(99)); expect_bad = 1; }                                      // unknown token
            const int rc = fg_program_result(p, name.c_str(), t.data(), (int)t.size());
            if (expect_bad) { if (rc != FG_E_BAD_ARG) return fail("a corrupted stream was not FG_E_BAD_ARG", rc); ++refused; continue; }
            if (rc != R) return fail("result index", rc);
            ++R; ++accepted;
            if (fg_program_result(p, name.c_str(), t.data(), (int)t.size()) != FG_E_BAD_ARG) return fail("duplicate name accepted", 0);
        }
        if (fg_program_result(p, "", npar, 1) != FG_E_BAD_ARG || fg_program_result(p, nullptr, npar, 1) != FG_E_BAD_ARG || fg_program_result(p, "x", nullptr, 1) != FG_E_BAD_ARG ||
            fg_program_result(p, "x", npar, 0) != FG_E_BAD_ARG) return fail("empty name / expression accepted", 0);
        int rc = fg_program_finalize(p);
        if (rc) return fail("finalize", rc);
        if (fg_program_result(p, "late", npar, 1) != FG_E_STATE) return fail("a result after finalize was not FG_E_STATE", 0);
        if (fg_program_n_results(p) != R) return fail("n_results", fg_program_n_results(p));
        for (int r = 0; r < R; ++r) {
            char small[4], buf[64];
            const int need = fg_program_result_name(p, r, buf, sizeof buf);
            if (need != (int)std::strlen(buf) + 1 || std::string(buf) != "result[" + std::to_string(r) + "]") return fail("result name", need);
            if (fg_program_result_name(p, r, small, sizeof small) != need || std::strlen(small) != 3) return fail("result name into a short buffer", 0);
        }
        if (fg_program_result_name(p, R, nullptr, 0) != FG_ERR_ADDRESS_NOT_FOUND || fg_program_result_name(p, -1, nullptr, 0) != FG_ERR_ADDRESS_NOT_FOUND) return fail("result name out of range", 0);
        std::vector<int32_t> sites((size_t)S + 1, -7);
        const int n_used = fg_program_result_sites(p, sites.data(), 1);      // a short buffer: one entry written, the count returned
        if (n_used < 0 || n_used > S || sites[1] != -7 || n_used != (int)p->res_sites.size()) return fail("result sites", n_used);
        if (fg_program_result_sites(p, sites.data(), S) != n_used) return fail("result sites (second call)", 0);
        if (R == 0 && (p->res_n_ins != 0 || n_used != 0)) return fail("a program without results has result instructions", p->res_n_ins);
        if (R > 0) { const char *w = walk(p); if (w) return fail(w, 0); }
        ++programs;
        fg_program_free(p);
    }
    std::printf("results ok %d refused %d programs %d\n", accepted, refused, programs);
    return 0;
}
