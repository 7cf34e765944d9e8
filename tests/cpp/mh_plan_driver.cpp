// The launch plan of the multi-wave MH kernels (fugue_amd/csrc/fg_mh_mw_plan.h) over a file of cases, as the launchers of fg_mh.hip
// put it together at an engine's first launch, for tests/test_mh_mw_plan_cpu.py (g++, no GPU).
//   mh_plan_driver variants     the keys of FG_MH_VARIANTS, one per line: pipe rk split
//   mh_plan_driver FILE         one line per case of FILE:
//       in:  no_stream C n_simd n_slots S mw_override has_overrides sstream_kinds sstream_gen n_pri n_ins_fast
//            17 switches ("u" = unset, else the integer): pipe exp split prio prio2 stagger catu jit gen_min gen_all nseg nseg_ns ctl16 bake jit_any jit_sums sums_form
//            site_vtype[S]  site_cat[2 S]  n_pool (pool entry as its 64 bits)*
//            a stream program:  n_rec = n_s + 2, (xi mi flags coord ximm mimm)* with the immediates as their 64 bits
//            a program without one:  n_stmt acc*
//       out: name=value,value,... fields (values are integers, doubles as their 64 bits), the kernel names last
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../fugue_amd/csrc/fg_mh_mw_plan.h"

template <typename It> static void put(const char *name, It a, It b) {
    std::cout << ' ' << name << '=';
    for (It q = a; q != b; ++q) std::cout << (q == a ? "" : ",") << (long long)*q;
}
static void put(const char *name, long long v) { put(name, &v, &v + 1); }
static double from_bits(unsigned long long b) { double d; std::memcpy(&d, &b, 8); return d; }

static void put_spec(const FgMhJitSpec &sp) {
    put("tried", sp.tried); put("unit", sp.unit);
    if (!sp.unit) return;
    put("generated", sp.generated.begin(), sp.generated.end()); put("rows", sp.rows.begin(), sp.rows.end());
    const int v[] = { sp.rk, sp.split, sp.n_pri, sp.n_fac, sp.no_stream, sp.pipe, sp.nseg, sp.ctl16, sp.sum_pri, sp.sum_lik, sp.bake, sp.bake_rows, sp.sums_form };
    put("spec", std::begin(v), std::end(v));
    if (sp.bake) put("baked", sp.baked, sp.baked + 7);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    if (std::string(argv[1]) == "variants") {
#define FG_PRINT_KEY(PIPE, RK, SPLIT) std::printf("%d %d %d\n", (int)PIPE, RK, (int)SPLIT);
        FG_MH_VARIANTS(FG_PRINT_KEY)
        return 0;
    }
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream s(line);
        FgMhPlanIn in{};
        int no_stream = 0, ov = 0;
        s >> no_stream >> in.C >> in.n_simd >> in.n_slots >> in.S >> in.mw_override >> ov >> in.sstream_kinds >> in.sstream_gen >> in.n_pri >> in.n_ins_fast;
        in.has_overrides = ov != 0;
        FgMhSwitches sw{};
        FgSwitch *swp[17] = { &sw.pipe, &sw.exp, &sw.split, &sw.prio, &sw.prio2, &sw.stagger, &sw.catu, &sw.jit, &sw.gen_min, &sw.gen_all, &sw.nseg, &sw.nseg_ns, &sw.ctl16,
                              &sw.bake, &sw.jit_any, &sw.jit_sums, &sw.sums_form };
        for (FgSwitch *w : swp) { std::string t; s >> t; w->set = t != "u"; w->v = w->set ? std::atoi(t.c_str()) : 0; }
        std::vector<int> vtype((size_t)in.S), cat(2 * (size_t)in.S);
        for (int &v : vtype) s >> v;
        for (int &v : cat) s >> v;
        size_t n = 0;
        s >> n;
        std::vector<double> pool(n);
        for (double &v : pool) { unsigned long long b; s >> b; v = from_bits(b); }
        s >> n;
        std::vector<FgGradRec> rec(no_stream ? 0 : n, FgGradRec{});
        std::vector<unsigned char> acc(no_stream ? n : 0);
        for (FgGradRec &r : rec) { unsigned long long a, b; s >> r.xi >> r.mi >> r.flags >> r.coord >> a >> b; r.ximm = from_bits(a); r.mimm = from_bits(b); }
        for (unsigned char &a : acc) { int v; s >> v; a = (unsigned char)v; }
        if (!s || (!no_stream && n < 2)) return 3;
        in.site_vtype = vtype.data(); in.site_cat = cat.data(); in.pool = &pool;
        FgMhMwShape sh;
        int rc;
        if (no_stream) {
            rc = fg_mh_mw_shape(in, (int)n, false, false, sw, sh);
            put("rc", rc);
        } else {
            in.sstream = rec.data(); in.n_s = (int)n - 2;
            const FgMhTail t = fg_mh_mw_tail(in, sw);
            const long long c0 = fg_mhp_bits(t.c0);
            std::vector<long long> cb, sites;
            for (double v : t.c) cb.push_back(fg_mhp_bits(v));
            for (const FgMhTailSite &q : t.sites) { sites.push_back(q.slot); sites.push_back(q.K); }
            rc = fg_mh_mw_shape(in, in.n_s - t.n_cu, in.sstream_kinds != 0, true, sw, sh);
            put("rc", rc); put("n_cu", t.n_cu); put("catu_same", t.same); put("catu_c0", c0); put("catu_c", cb.begin(), cb.end()); put("catu", sites.begin(), sites.end());
        }
        if (rc == FG_OK) {
            const long long shape[] = { (long long)sh.lds, sh.W, sh.exp_mask, sh.split_sums, sh.pool_n, sh.pipe, sh.resident, (long long)sh.tiles };
            put("shape", std::begin(shape), std::end(shape));
            if (no_stream) put_spec(fg_mh_mw_jit_spec_nostream(in, sh, acc, (int)n, sw));
            else {
                const int n_cu = fg_mh_mw_tail(in, sw).n_cu;
                int cls_off[FG_MHP_NCLS + 1], r[FG_MHP_NCLS][FG_MHP_WMAX + 1];
                const std::vector<int> order = fg_mh_mw_order(in, n_cu, cls_off);
                std::vector<int> coord;
                for (int k : order) coord.push_back(fg_mh_mw_row(in, n_cu, k));
                fg_mh_mw_segments(cls_off, sh, r);
                put("cls_off", cls_off, cls_off + FG_MHP_NCLS + 1); put("order", order.begin(), order.end()); put("coord", coord.begin(), coord.end());
                put("seg_r", &r[0][0], &r[0][0] + FG_MHP_NCLS * (FG_MHP_WMAX + 1));
                put_spec(fg_mh_mw_jit_spec(in, sh, n_cu, cls_off, sw));
                const FgMhMwKey key = fg_mh_mw_key(in, sh);
                const int kv[] = { key.pipe, key.rk, key.split };
                put("key", kv, kv + 3);
            }
            std::cout << " name=" << fg_mh_mw_name(sh, false, no_stream != 0) << "|" << fg_mh_mw_name(sh, true, no_stream != 0);
        }
        std::cout << '\n';
    }
    return 0;
}
