// The plans of fugue_amd/csrc/fg_hmc_split_plan.h over a file of cases, for tests/test_hmc_split_plan_cpu.py (g++, no GPU).
//   split_plan_driver FILE       one JSON line per case of FILE; a switch is "u" (unset) or its integer; a coordinate's sub-program is
//                                four counts: hoisted densities, general densities, fast Normals, plain operations
//     cost OP OPND1                                       fg_task_ins_cost of one instruction
//     jit d S n_simd mw  tiles0 waves0 jocc0 fused0 tasks0  tiles waves jocc fused mode has_ad  (4 counts) x d
//                                                         the unit generated at tiles0 under the first switches, then prepared and launched at
//                                                         `tiles` under the second in gradient mode `mode` (FG_JIT_VERBOSE set throughout)
//     mwi d S n_slots mw n_simd tiles prog_bytes mode  waves occ ldsprog  tiles2 waves2 occ2 ldsprog2  (4 counts) x d
//                                                         the interpreter kernel's first launch, then a second one on the same engine
//     stream d tiles n_simd lds_bytes mw tw gt mode sstream_kinds has_ss nrec  (coord flags maskm xi mi) x nrec
//     first                                               fg_hmc_jit_first over mode x jit_state x gstream x gt x tw x sep gate x lin gate
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../fugue_amd/csrc/fg_hmc_split_plan.h"

typedef std::vector<std::vector<int>> Bins;
struct JitCase { int d, S, n_simd, mw; unsigned tiles[2]; FgSwitch waves[2], jocc[2], fused[2], tasks; int mode, has_ad; std::vector<FgCoord> coord; std::vector<FgIns> sub; };
struct JitOut { Bins gbins, gcb, gcbd, cb; int W; std::vector<int> off, off_an, off_used, order; std::string say, name; int baked, fused; long long lds, lds_eps; };
struct MwiCase { int d, S, n_slots, mw, n_simd, mode; unsigned tiles[2]; size_t prog_bytes; FgSwitch waves[2], occ[2], ldsprog[2]; std::vector<FgCoord> coord; std::vector<FgIns> sub; };
struct MwiOut { int rc, W; std::vector<int> off, order; int occ[2], pl[2]; long long lds[2]; std::string name[2]; };
struct StreamCase { int d, n_simd, mw, tw, gt, mode, sstream_kinds, has_ss; unsigned tiles; size_t lds_bytes; std::vector<FgGradRec> gs; };
struct StreamOut { int rc, W; std::vector<int> c, g; int separable, rk, an, ss; std::string name; };

static FgSwitch sw_of(std::istream &s) { std::string t; s >> t; return FgSwitch{ t != "u", t != "u" ? std::atoi(t.c_str()) : 0 }; }
static void subs_of(std::istream &s, int d, std::vector<FgCoord> &coord, std::vector<FgIns> &sub) {
    const uint32_t ops[4] = { 0u | FG_F_HOISTED, 3u, FG_OP_NORMAL_FAST, FG_OP_ADD };
    for (int k = 0; k < d; ++k) {
        FgCoord c = { k, (int)sub.size(), 0, 0 };
        for (uint32_t op : ops) { int n = 0; s >> n; for (int q = 0; q < n; ++q) { FgIns in = FgIns(); in.op = op; sub.push_back(in); } }
        c.sub_n = (int)sub.size() - c.sub_off;
        coord.push_back(c);
    }
}
static void put(const char *k, long long v) { std::cout << '"' << k << "\":" << v << ','; }
static void put(const char *k, const std::string &v) { std::cout << '"' << k << "\":\""; for (char c : v) { if (c == '\n') std::cout << "\\n"; else std::cout << c; } std::cout << "\","; }
static void put(const char *k, const std::vector<int> &v) { std::cout << '"' << k << "\":["; for (size_t i = 0; i < v.size(); ++i) std::cout << (i ? "," : "") << v[i]; std::cout << "],"; }
static void put(const char *k, const Bins &v) {
    std::cout << '"' << k << "\":[";
    for (size_t w = 0; w < v.size(); ++w) { std::cout << (w ? ",[" : "["); for (size_t i = 0; i < v[w].size(); ++i) std::cout << (i ? "," : "") << v[w][i]; std::cout << ']'; }
    std::cout << "],";
}

// ---- evaluation: the plans as the launchers (fg_hmc_interp.hip, fg_engine.hip) compose them ---------------------------------------------------
static Bins bins_of(const FgTaskSplit &s, int n_tasks) {
    Bins b;
    for (int w = 0; w < s.W; ++w) b.emplace_back(s.order.begin() + s.off[w], s.order.begin() + std::min(s.off[w + 1], n_tasks));
    return b;
}
static long long eval_cost(const FgIns &in) { return fg_task_ins_cost(in); }
static JitOut eval_jit(const JitCase &c) {
    JitOut o;
    std::vector<long long> cost, tcost;
    fg_task_coord_costs(c.coord.data(), c.d, c.sub.data(), cost, tcost);
    FgTaskSwitches sw = FgTaskSwitches();
    sw.verbose = FgSwitch{ true, 1 };
    FgTaskSplit gen[2];
    for (int dense = 0; dense < 2 && !fg_switch_is(c.tasks, 0); ++dense) {        // jit_hmc_module
        sw.waves = c.waves[0]; sw.jit_occ = c.jocc[0]; sw.fused = c.fused[0]; sw.tasks = c.tasks;
        const FgJitTaskIn in = { c.d, c.S, c.tiles[0], c.n_simd, c.mw, &cost, &tcost, dense ? FG_GRAD_FD_DENSE : FG_GRAD_FD_SPARSE, sw };
        gen[dense] = fg_jit_task_plan(in).split;
    }
    o.gbins = bins_of(gen[0], 2 * c.d); o.gcb = gen[0].cbins; o.gcbd = gen[1].cbins;
    sw.waves = c.waves[1]; sw.jit_occ = c.jocc[1]; sw.fused = c.fused[1];         // jit_hmc_prepare
    const FgJitTaskIn in = { c.d, c.S, c.tiles[1], c.n_simd, c.mw, &cost, &tcost, c.mode, sw };
    const FgJitTaskPlan p = fg_jit_task_plan(in);
    o.W = p.split.W; o.off.assign(p.split.off, p.split.off + 17); o.off_an.assign(p.split.off_an, p.split.off_an + 17); o.order = p.split.order; o.cb = p.split.cbins;
    o.say = fg_jit_task_say(p, c.d);
    const FgJitLaunchShape sh = fg_jit_launch_shape(p.split, gen[c.mode == FG_GRAD_FD_DENSE], c.mode, c.has_ad != 0, c.S, c.d);   // fg_hmc_jit_launch
    o.baked = sh.baked; o.fused = sh.fused; o.lds = (long long)sh.lds; o.name = sh.name; o.off_used = sh.analytic_off ? o.off_an : o.off;
    o.lds_eps = fg_task_lds(c.S, c.d, p.split.W);                                 // fg_hmc_jit_find_eps
    return o;
}
static MwiOut eval_mwi(const MwiCase &c) {
    MwiOut o = MwiOut();
    FgTaskSplit split;
    for (int q = 0; q < 2; ++q) {                                                 // two launches of one engine: the split is the first one's
        FgTaskSwitches sw = FgTaskSwitches();
        sw.waves = c.waves[q]; sw.occ = c.occ[q]; sw.ldsprog = c.ldsprog[q];
        if (q == 0) {
            std::vector<long long> cost((size_t)c.d, 1), tcost;
            if (c.mode != FG_GRAD_FD_DENSE) fg_task_coord_costs(c.coord.data(), c.d, c.sub.data(), cost, tcost);
            const FgMwiTaskIn in = { c.d, c.S, c.n_slots, c.mw, &cost, sw };
            if ((o.rc = fg_mwi_task_plan(in, &split)) != FG_OK) return o;
            o.W = split.W; o.off.assign(split.off, split.off + 17); o.order = split.order;
        }
        const FgMwiLaunchIn lin = { c.d, c.S, c.n_slots, split.W, c.prog_bytes, c.tiles[q], c.n_simd, sw };
        const FgMwiLaunchShape sh = fg_mwi_launch_shape(lin);
        o.occ[q] = sh.occ; o.pl[q] = sh.pl; o.lds[q] = (long long)sh.lds; o.name[q] = sh.name;
    }
    return o;
}
static StreamOut eval_stream(const StreamCase &c) {
    StreamOut o = StreamOut();
    const FgStreamPlanIn in = { c.d, c.tiles, c.n_simd, c.lds_bytes, c.mw, c.tw, c.gt != 0, c.gs.empty() ? nullptr : c.gs.data(), (int)c.gs.size(), c.sstream_kinds, c.has_ss != 0, c.mode };
    FgStreamPlan p;
    if ((o.rc = fg_hmc_stream_plan(in, &p)) != FG_OK) return o;
    o.W = p.W; o.c.assign(p.c, p.c + 17); o.g.assign(p.g, p.g + 17); o.separable = p.separable; o.rk = p.rk; o.an = p.analytic; o.ss = p.ss; o.name = p.name;
    return o;
}
static bool eval_first(int mode, int jit_state, bool gstream, bool gt, int tw, bool sep_gate, bool lin_gate) {
    const FgJitFirstIn in = { mode, jit_state, gstream, gt, tw, sep_gate, lin_gate };
    return fg_hmc_jit_first(in);
}
// ---- end of evaluation ------------------------------------------------------------------------------------------------------------------------

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream s(line);
        std::string kind;
        s >> kind;
        std::cout << '{';
        if (kind == "cost") {
            FgIns in = FgIns();
            s >> in.op >> in.opnd[1];
            put("cost", eval_cost(in));
        } else if (kind == "jit") {
            JitCase c;
            s >> c.d >> c.S >> c.n_simd >> c.mw >> c.tiles[0];
            c.waves[0] = sw_of(s); c.jocc[0] = sw_of(s); c.fused[0] = sw_of(s); c.tasks = sw_of(s);
            s >> c.tiles[1];
            c.waves[1] = sw_of(s); c.jocc[1] = sw_of(s); c.fused[1] = sw_of(s);
            s >> c.mode >> c.has_ad;
            subs_of(s, c.d, c.coord, c.sub);
            const JitOut o = eval_jit(c);
            put("gbins", o.gbins); put("gcb", o.gcb); put("gcbd", o.gcbd); put("W", o.W); put("off", o.off); put("off_an", o.off_an); put("off_used", o.off_used); put("order", o.order); put("cb", o.cb);
            put("say", o.say); put("baked", o.baked); put("fused", o.fused); put("lds", o.lds); put("lds_eps", o.lds_eps); put("name", o.name);
        } else if (kind == "mwi") {
            MwiCase c;
            s >> c.d >> c.S >> c.n_slots >> c.mw >> c.n_simd >> c.tiles[0] >> c.prog_bytes >> c.mode;
            c.waves[0] = sw_of(s); c.occ[0] = sw_of(s); c.ldsprog[0] = sw_of(s);
            s >> c.tiles[1];
            c.waves[1] = sw_of(s); c.occ[1] = sw_of(s); c.ldsprog[1] = sw_of(s);
            subs_of(s, c.d, c.coord, c.sub);
            const MwiOut o = eval_mwi(c);
            put("rc", o.rc);
            if (o.rc == FG_OK) {
                put("W", o.W); put("off", o.off); put("order", o.order);
                for (int q = 0; q < 2; ++q) { put(q ? "occ2" : "occ", o.occ[q]); put(q ? "pl2" : "pl", o.pl[q]); put(q ? "lds2" : "lds", o.lds[q]); put(q ? "name2" : "name", o.name[q]); }
            }
        } else if (kind == "stream") {
            StreamCase c;
            size_t nrec = 0;
            s >> c.d >> c.tiles >> c.n_simd >> c.lds_bytes >> c.mw >> c.tw >> c.gt >> c.mode >> c.sstream_kinds >> c.has_ss >> nrec;
            c.gs.assign(nrec, FgGradRec());
            for (FgGradRec &r : c.gs) s >> r.coord >> r.flags >> r.maskm >> r.xi >> r.mi;
            const StreamOut o = eval_stream(c);
            put("rc", o.rc);
            if (o.rc == FG_OK) { put("W", o.W); put("c", o.c); put("g", o.g); put("separable", o.separable); put("rk", o.rk); put("an", o.an); put("ss", o.ss); put("name", o.name); }
        } else if (kind == "first") {
            std::string t;
            const int modes[3] = { FG_GRAD_FD_DENSE, FG_GRAD_FD_SPARSE, FG_GRAD_ANALYTIC };
            for (int mode : modes) for (int js = -1; js <= 1; ++js) for (int b = 0; b < 32; ++b)
                t += eval_first(mode, js, (b & 1) != 0, (b & 2) != 0, (b & 4) ? 32 : 64, (b & 8) != 0, (b & 16) != 0) ? '1' : '0';
            put("first", t);
        } else return 3;
        if (!s) return 3;
        std::cout << "\"kind\":\"" << kind << "\"}\n";
    }
    return 0;
}
