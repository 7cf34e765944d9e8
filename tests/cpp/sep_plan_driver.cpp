// fg_hmc_sep_plan (fugue_amd/csrc/fg_hmc_sep_plan.h) over a file of cases, for tests/test_hmc_sep_plan_cpu.py (g++, no GPU).
//   sep_plan_driver variants     the keys of FG_SEP_VARIANTS, one per line: mass mode half nc nobs u0 fold
//   sep_plan_driver FILE         one line per case of FILE:
//       in:  C d n_simd n_slots n_sep_free n_sstream grad_mode use_mass mw_override gt sep_disabled res_disabled fold_disabled sep_fold
//            6 switches ("u" = unset, else the integer)  n_coord (off n)*  n_rec trow*
//       out: rc [half tw tiles W lds  key(7)  c(17)  sum4 predraw  n_own(16)  own(64)  name]
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../fugue_amd/csrc/fg_hmc_sep_plan.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    if (std::string(argv[1]) == "variants") {
#define FG_PRINT_KEY(M, MODE, HALF, NC, NOBS, U0, FOLD) std::printf("%d %d %d %d %d %d %d\n", (int)M, MODE, HALF, NC, NOBS, (int)U0, (int)FOLD);
        FG_SEP_VARIANTS(FG_PRINT_KEY)
        return 0;
    }
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream s(line);
        FgSepPlanIn in{};
        int flag[6];
        s >> in.C >> in.d >> in.n_simd >> in.n_slots >> in.n_sep_free >> in.n_sstream >> in.grad_mode >> flag[0] >> in.mw_override >> flag[1] >> flag[2] >> flag[3] >> flag[4] >> flag[5];
        in.use_mass = flag[0]; in.gt = flag[1]; in.sep_disabled = flag[2]; in.res_disabled = flag[3]; in.fold_disabled = flag[4]; in.sep_fold = flag[5];
        FgSwitch *sw[6] = { &in.sep_half, &in.dense_fast, &in.sum4, &in.prio, &in.stagger, &in.predraw };
        for (FgSwitch *w : sw) { std::string t; s >> t; w->set = t != "u"; w->v = w->set ? std::atoi(t.c_str()) : 0; }
        size_t n = 0;
        s >> n;
        std::vector<FgSepCoord> coord(n);
        for (FgSepCoord &q : coord) s >> q.off >> q.n;
        s >> n;
        std::vector<FgSepRec> rec(n, FgSepRec{});
        for (FgSepRec &q : rec) s >> q.trow;
        if (!s) return 3;
        in.coord = &coord; in.rec = &rec;
        FgSepPlan p;
        const int rc = fg_hmc_sep_plan(in, &p);
        std::cout << rc;
        if (rc == FG_OK) {
            std::cout << ' ' << p.half << ' ' << p.tw << ' ' << p.tiles << ' ' << p.W << ' ' << p.lds << ' ' << p.key.mass << ' ' << p.key.mode << ' ' << p.key.half << ' '
                      << p.key.nc << ' ' << p.key.nobs << ' ' << p.key.u0 << ' ' << p.key.fold;
            for (int v : p.seg.c) std::cout << ' ' << v;
            std::cout << ' ' << p.seg.sum4 << ' ' << p.seg.predraw;
            for (int v : p.seg.n_own) std::cout << ' ' << v;
            for (const auto &row : p.seg.own) for (int v : row) std::cout << ' ' << v;
            std::cout << ' ' << p.name;
        }
        std::cout << '\n';
    }
    return 0;
}
